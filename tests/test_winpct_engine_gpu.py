"""The wp stream through the whole engine: parse -> device join -> K7 -> K8 -> K16, against
PipelineOracle over several rollovers; with lh on as well; the other streams unchanged by it; the
engine's resources returned.  (Shapes of tests/test_hist_engine_gpu.py.)"""
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
from apmbackend_amd.models.pipeline import ALL_OUT_KINDS, OUT_KINDS, APMEngine  # noqa: E402
from test_hist_engine_gpu import KINDS, UTC, run, small_cfg, synth_batches  # noqa: E402

PCTS = [50, 90, 99, 99.9]


def pct_cfg(lh=False):
    C = small_cfg()
    C["gpu"]["windowPercentiles"] = list(PCTS)
    if lh:
        C["gpu"]["latencyHistogram"] = True
    return C


def test_stream_is_opt_in():
    assert ALL_OUT_KINDS == OUT_KINDS + ("wp",)
    eng = APMEngine(pct_cfg(), keep_text=True)   # a list in the config alone does not start it
    assert not (eng.ecfg["outputs"] >> ALL_OUT_KINDS.index("wp")) & 1
    with pytest.raises(ValueError):
        APMEngine(small_cfg(), outputs=("st", "wp"))
    bad = small_cfg()
    bad["gpu"]["windowPercentiles"] = [99, 50]
    with pytest.raises(ValueError):
        APMEngine(bad, outputs=("st", "wp"))
    # the native constructor checks the list it is handed as well
    N = _native.load()
    from apmbackend_amd.models.pipeline import engine_config
    ecfg = engine_config(pct_cfg(), outputs=("st", "wp"))
    for lst in ([], [50000, 50000], [0], [100001], list(range(1, 10))):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, win_pcts=lst))


def test_full_pipeline_matches_oracle_and_changes_nothing_else():
    _lines, bl = synth_batches(seed=1, duration=300)
    C = pct_cfg()
    kinds = KINDS + ("wp",)
    _e, on = run(C, bl, kinds, kinds=kinds)
    _e, off = run(small_cfg(), bl, KINDS, kinds=KINDS + ("wp",))
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert len(P.wp) > 100
    assert on["wp"] == P.wp
    assert off["wp"] == []   # as take("lh") with lh off
    for k in ("st", "fs", "al", "audit_db", "transactions"):
        assert on[k] == off[k], k
    assert collections.Counter(on["db"]) == collections.Counter(off["db"]) and len(on["db"]) > 100
    assert on["st"] == P.stats
    # one row per st row whose window holds a sample, in st order, with its timestamp
    st_keys = [tuple(l.split("|")[1:4]) for l in on["st"] if l.split("|")[5] != "undefined"]
    assert [tuple(l.split("|")[1:4]) for l in on["wp"]] == st_keys
    assert all(l.split("|")[6].split(",")[0].startswith("50:") and ",99.9:" in l for l in on["wp"])


def test_with_the_histogram_stream_on_both_are_right():
    _lines, bl = synth_batches(seed=5, duration=200)
    C = pct_cfg(lh=True)
    kinds = KINDS + ("lh", "wp")
    _e, on = run(C, bl, kinds, kinds=kinds)
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert len(P.wp) > 50 and len(P.lh) > 50
    assert on["wp"] == P.wp and on["lh"] == P.lh and on["st"] == P.stats


def test_resources_return_after_the_engine():
    COUNTS = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes", "events", "streams")
    gc.collect()
    N = _native.load()
    before = dict(N.live_resources())
    _lines, bl = synth_batches(seed=3, duration=150)
    kinds = KINDS + ("wp",)
    eng, out = run(pct_cfg(), bl, kinds, kinds=kinds)
    assert len(out["wp"]) > 10
    during = dict(N.live_resources())
    assert during["device_bytes"] - before["device_bytes"] == eng.eng.device_bytes()
    del eng, out
    gc.collect()
    after = dict(N.live_resources())
    assert {k: after[k] for k in COUNTS} == {k: before[k] for k in COUNTS}
